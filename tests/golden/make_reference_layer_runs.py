#!/usr/bin/env python3
"""Record what the reference's own Python layers compute over this repository's fused operator -> ``reference_layer_runs.json``.

Usage: ``python tests/golden/make_reference_layer_runs.py <reference checkout>`` (the directory that holds the ``gpytorch`` package).

The reference package imports the third-party ``linear_operator`` package, which is not installed: ``tests/shim/linear_operator`` maps every
name it imports onto the class of the same role in ``gpytorch_amd.operators`` / ``gpytorch_amd.settings``, and
``gpytorch_amd.dropin.build(gpytorch, linear_operator)`` yields plugin kernels whose ``forward`` returns the fused operator.  For every case
of ``tests/test_reference_layers_cpu.py`` the reference's own ExactGP + GaussianLikelihood + ExactMarginalLogLikelihood then run forward,
backward and in eval mode (exact and ``fast_pred_var`` variances) over the plugin, on the CPU double of the native entry points
(``tests/shim/cpu_backend.py``).  Recorded per case: the MLL value, the raw-parameter gradients, the predictive mean and both variances, how
often the fused operator's entry points were called, and which functions of which files of the reference executed.  The JSON holds numbers
and names only; the test compares this repository's standalone layers with it.
"""
from __future__ import annotations

import importlib
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_reference_layers_cpu import CASES, GOLDEN, HP, SHIM, _data, _run, case_key  # noqa: E402


class FileTrace:
    """Records which files of the reference had a function executed (``sys.setprofile``: call events only)."""

    def __init__(self, ref):
        self.prefix, self.files = os.path.join(ref, "gpytorch") + os.sep, {}

    def __call__(self, frame, event, arg):
        if event == "call":
            fn = frame.f_code.co_filename
            if fn.startswith(self.prefix):
                self.files.setdefault("gpytorch/" + fn[len(self.prefix):], set()).add(frame.f_code.co_name)

    def __enter__(self):
        sys.setprofile(self)
        return self

    def __exit__(self, *exc):
        sys.setprofile(None)


def record_case(ref, kind, nu, lazy):
    from gpytorch_amd import dropin
    from gpytorch_amd import operators as own_ops
    from tests.shim import cpu_backend

    with pytest.MonkeyPatch.context() as mp:
        cpu_backend.install(mp)
        mp.syspath_prepend(ref)
        mp.syspath_prepend(SHIM)
        before = set(sys.modules)
        try:
            lo = importlib.import_module("linear_operator")
            gp = importlib.import_module("gpytorch")
            assert gp.__file__.startswith(ref) and lo.__file__.startswith(SHIM)
            ns = dropin.build(gp, lo)
            calls = {"inv_quad_logdet": 0, "solve": 0, "root_inv_decomposition": 0}
            for name in calls:     # the FUSED operator's entry points must be what the reference's layers end up calling
                orig = getattr(own_ops.FusedKernelAddedDiagLinearOperator, name)

                def spy(self, *a, _orig=orig, _name=name, **kw):
                    calls[_name] += 1
                    return _orig(self, *a, **kw)

                mp.setattr(own_ops.FusedKernelAddedDiagLinearOperator, name, spy)
            X, y, Xs = _data()
            kern = ns.RBFKernel if nu is None else (lambda: ns.MaternKernel(nu=nu))
            with FileTrace(ref) as tr:
                v, g, mu, var, love = _run(gp, kern, X, y, Xs, HP, lambda: gp.settings.lazily_evaluate_kernels(lazy))
            # the classes that ran are the reference's own, and the operator under them is the plugin
            assert gp.mlls.ExactMarginalLogLikelihood.__module__ == "gpytorch.mlls.exact_marginal_log_likelihood"
            assert ns.ExactMarginalLogLikelihood is gp.mlls.ExactMarginalLogLikelihood
        finally:
            for name in set(sys.modules) - before:
                if name.split(".")[0] in ("gpytorch", "linear_operator"):
                    del sys.modules[name]
    return {
        "mll": v,
        "grads": {k: t.tolist() for k, t in sorted(g.items())},
        "mean": mu.tolist(),
        "variance": var.tolist(),
        "variance_fast_pred_var": love.tolist(),
        "fused_operator_entry_points_called": calls,
        "executed": {f: sorted(fns) for f, fns in sorted(tr.files.items())},
    }


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "gpytorch")):
        sys.exit(__doc__.split("\n\n")[1])
    ref = os.path.abspath(sys.argv[1])
    doc = {
        "what": "the reference's ExactGP + GaussianLikelihood + ExactMarginalLogLikelihood (forward, backward) and DefaultPredictionStrategy (mean, "
                "exact and fast_pred_var variance) run over gpytorch_amd.dropin's plugin kernel / operator on tests/test_reference_layers_cpu.py's "
                "data (n = 300 <= max_cholesky_size, float32, native entry points doubled on the CPU by tests/shim/cpu_backend.py); "
                "written by tests/golden/make_reference_layer_runs.py",
        "hyperparameters": dict(zip(("lengthscale", "outputscale", "noise", "constant_mean"), HP)),
        "cases": {case_key(kind, lazy): record_case(ref, kind, nu, lazy) for kind, nu in CASES for lazy in (False, True)},
    }
    with open(GOLDEN, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {GOLDEN}")


if __name__ == "__main__":
    main()
