"""Old against new for the structured "K + diagonal" operators: the same model per operator, evaluated by the parent commit's Python package and by
this tree's, on the SAME libgpamd.so -- values, solver iterations and the wall time of an MLL forward + backward.

    python scripts/added_diag_ab.py --export [REV]     where the repository is: REV's gpytorch_amd/ -> gpu_jobs/parent/ (git archive; default HEAD,
                                                       the parent while the change is uncommitted -- HEAD~1 once it is committed)
    python scripts/added_diag_ab.py [--ops sum,hadamard,kronecker,grad,ski] [--rounds 2] [--out profiles/added_diag_refactor_ab.json]
    python scripts/added_diag_ab.py --child OP FILE    (what the driver starts: one side, one operator, results to FILE)

The driver starts every measurement as a fresh child process (PYTHONPATH picks the side, GPAMD_LIBRARY the one library), sides alternating, each
child under its own time limit; the first child that fails ends the run.  Per operator and side it records inv_quad, logdet, every
hyper-parameter gradient, the CG iteration count of the MLL (``bbmm_opts["_last_info"]``), one solve, one product with the Lanczos root of the
inverse, and the times of ``--reps`` MLL forward + backward passes, each ended by a device synchronise.  Probes are ``settings.deterministic_probes``
under a fixed seed.  Expected: iteration counts identical, values bitwise equal (no arithmetic moved); where the parent does not reproduce itself
bit by bit between two of its own runs, the parent-to-new difference has to stay within the parent-to-parent one.  Time: the new median inside
the range of the parent's own samples of the same call."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT = os.path.join(ROOT, "gpu_jobs", "parent")
LIB = os.path.join(ROOT, "gpytorch_amd", "csrc", "libgpamd.so")
OPS = ("sum", "hadamard", "kronecker", "grad", "ski")
# sizes a user would run: (points, input dimensions)
SIZES = {"sum": (20_000, 3), "hadamard": (20_000, 2), "kronecker": (5_000, 2), "grad": (5_000, 2), "ski": (100_000, 2)}
TASKS = {"hadamard": 2, "kronecker": 4}
SKI_GRID = (100, 100)


# ---------------------------------------------------------------------------------------------------------------- one side, one operator
def _build(name, g, dev):
    """(modules holding the hyper-parameters, a function that builds the added-diagonal operator from them, the number of rows)."""
    import torch

    n, d = SIZES[name]
    gen = torch.Generator().manual_seed(0)
    x = (0.01 + 0.98 * torch.rand(n, d, generator=gen)).to(dev)
    lik = g.likelihoods.GaussianLikelihood().to(dev)
    lik.noise = 0.1
    if name == "sum":
        kern = (g.kernels.ScaleKernel(g.kernels.RBFKernel()) + g.kernels.ScaleKernel(g.kernels.MaternKernel(nu=2.5))).to(dev)
        ka, kb = kern.kernels
        ka.base_kernel.lengthscale, ka.outputscale = 0.25, 1.1
        kb.base_kernel.lengthscale, kb.outputscale = 0.9, 0.4
        return [kern, lik], (lambda: kern(x).evaluate_kernel().add_diagonal(lik.noise)), n
    if name == "hadamard":
        T = TASKS[name]
        tasks = torch.randint(0, T, (n,), generator=gen).to(dev)
        kx = g.kernels.RBFKernel().to(dev)
        kx.lengthscale = 0.35
        kt = g.kernels.IndexKernel(num_tasks=T, rank=1).to(dev)
        with torch.no_grad():
            kt.covar_factor.copy_(torch.tensor([[0.9], [-0.4]]))
        kt.var = torch.tensor([0.3, 0.5])
        return [kx, kt, lik], (lambda: kx(x).evaluate_kernel().mul(kt(tasks)).add_diagonal(lik.noise)), n
    if name == "kronecker":
        from gpytorch_amd.multitask import TaskNoiseDiagLinearOperator

        T = TASKS[name]
        kern = g.kernels.MultitaskKernel(g.kernels.RBFKernel(), num_tasks=T, rank=1).to(dev)
        kern.data_covar_module.lengthscale = 0.35
        with torch.no_grad():
            kern.task_covar_module.covar_factor.copy_(torch.tensor([[0.9], [-0.5], [0.7], [0.2]]))
        kern.task_covar_module.var = torch.tensor([0.4, 0.6, 0.3, 0.5])
        mlik = g.likelihoods.MultitaskGaussianLikelihood(num_tasks=T, has_global_noise=False).to(dev)
        mlik.task_noises = torch.tensor([0.05, 0.1, 0.08, 0.12])
        return [kern, mlik], (lambda: kern(x).evaluate_kernel() + TaskNoiseDiagLinearOperator(mlik._task_noise_vector(), n)), n * T
    if name == "grad":
        kern = g.kernels.ScaleKernel(g.kernels.RBFKernelGrad()).to(dev)
        kern.base_kernel.lengthscale, kern.outputscale = 0.35, 1.3
        return [kern, lik], (lambda: kern(x).evaluate_kernel().add_diagonal(lik.noise)), n * (d + 1)
    kern = g.kernels.ScaleKernel(g.kernels.GridInterpolationKernel(g.kernels.RBFKernel(), grid_size=list(SKI_GRID), grid_bounds=[(0.0, 1.0)] * d)).to(dev)
    kern.base_kernel.base_kernel.lengthscale, kern.outputscale = 0.3, 1.3
    return [kern, lik], (lambda: kern(x).evaluate_kernel().add_diagonal(lik.noise)), n


def child(name: str, out: str, reps: int) -> None:
    import torch

    import gpytorch_amd as g

    want = os.environ["ADDED_DIAG_AB_ROOT"]
    assert os.path.dirname(os.path.dirname(os.path.abspath(g.__file__))) == os.path.abspath(want), (g.__file__, want)
    assert torch.cuda.is_available(), "the comparison needs the device"
    dev = torch.device("cuda:0")
    S = g.settings
    modules, build, rows = _build(name, g, dev)
    params = {}
    for i, m in enumerate(modules):
        for k, p in m.named_parameters():
            params[f"{i}.{k}"] = p
    y = torch.randn(rows, 1, generator=torch.Generator().manual_seed(1)).to(dev)

    def mll():
        for p in params.values():
            p.grad = None
        op = build()
        iq, ld = op.inv_quad_logdet(y, logdet=True)
        (iq + ld).backward()
        torch.cuda.synchronize()
        return op, iq, ld

    rec = {}
    with S.deterministic_probes(True):
        torch.manual_seed(0)
        op, iq, ld = mll()                                               # (also the warm-up: code objects, the stored probe matrix)
        rec["inv_quad"], rec["logdet"] = iq.detach().cpu(), ld.detach().cpu()
        for k, p in params.items():
            if p.grad is not None:
                rec["grad:" + k] = p.grad.detach().cpu().clone()
        iterations = int(op.bbmm_opts["_last_info"].iterations)
        mll()
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            mll()
            times.append(time.perf_counter() - t0)
        with torch.no_grad(), S.cg_tolerance(0.01):
            torch.manual_seed(1)
            rec["solve"] = build().solve(y).cpu()
            torch.manual_seed(2)
            root = build().root_inv_decomposition().root
            rec["root_inv_product"] = (root @ (root.mT @ y)).cpu()
    torch.save({"values": rec, "iterations": iterations, "times": times, "rows": rows, "rank": int(root.shape[-1])}, out)


# ---------------------------------------------------------------------------------------------------------------- the driver
def export(rev: str) -> None:
    os.makedirs(PARENT, exist_ok=True)
    arch = subprocess.Popen(["git", "-C", ROOT, "archive", rev, "gpytorch_amd"], stdout=subprocess.PIPE)
    subprocess.run(["tar", "-x", "-C", PARENT, "--exclude=gpytorch_amd/csrc"], stdin=arch.stdout, check=True)
    if arch.wait() != 0:
        raise SystemExit("git archive failed")
    sha = subprocess.run(["git", "-C", ROOT, "rev-parse", rev], check=True, capture_output=True, text=True).stdout.strip()
    with open(os.path.join(PARENT, "REV"), "w") as f:
        f.write(sha + "\n")
    print("exported", sha, "to", PARENT)


def _diff(a: dict, b: dict) -> dict:
    """Per quantity: bitwise equality and the largest absolute / relative (to the largest entry) difference."""
    import torch

    out = {}
    assert a.keys() == b.keys(), (sorted(a), sorted(b))
    for k in a:
        d = float((a[k].double() - b[k].double()).abs().max()) if a[k].numel() else 0.0
        out[k] = {"bitwise": bool(torch.equal(a[k], b[k])), "max_abs": d, "max_rel": d / max(float(b[k].double().abs().max()), 1e-300) if a[k].numel() else 0.0}
    return out


def drive(ops, rounds: int, reps: int, out: str, limit: int) -> int:
    import torch

    if not os.path.isdir(os.path.join(PARENT, "gpytorch_amd")):
        raise SystemExit(f"{PARENT}/gpytorch_amd is missing: run --export where the repository is")
    if not os.path.exists(LIB):
        raise SystemExit(f"{LIB} is missing: build first")
    tmp = tempfile.mkdtemp(prefix="added_diag_ab_")                              # the children's result files; only the report is kept
    sides = {"parent": PARENT, "new": ROOT}
    report = {"parent_rev": open(os.path.join(PARENT, "REV")).read().strip() if os.path.exists(os.path.join(PARENT, "REV")) else None,
              "sizes": {k: {"points": SIZES[k][0], "d": SIZES[k][1], "tasks": TASKS.get(k)} for k in ops}, "ski_grid": list(SKI_GRID),
              "rounds": rounds, "reps": reps, "operators": {}}
    ok = True
    for name in ops:
        runs = {s: [] for s in sides}
        for r in range(rounds):
            for side in (("parent", "new") if r % 2 == 0 else ("new", "parent")):
                f = os.path.join(tmp, f"{name}_{side}_{r}.pt")
                env = dict(os.environ, PYTHONPATH=sides[side], GPAMD_LIBRARY=LIB, ADDED_DIAG_AB_ROOT=sides[side])
                print(f"[{name}] round {r} {side} ...", flush=True)
                try:
                    rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, f, "--reps", str(reps)], env=env, cwd=tmp,
                                        timeout=limit).returncode
                except subprocess.TimeoutExpired:
                    rc = 124
                if rc != 0:                                                  # nothing more is started on the device after a failure
                    print(f"[{name}] {side} round {r}: exit status {rc}; stopping", flush=True)
                    report["stopped"] = {"operator": name, "side": side, "round": r, "exit_status": rc}
                    with open(out, "w") as fh:
                        json.dump(report, fh, indent=1)
                    return 1
                runs[side].append(torch.load(f))
        p, q = runs["parent"], runs["new"]
        new_vs_parent = [_diff(q[r]["values"], p[r]["values"]) for r in range(rounds)]
        parent_vs_parent = [_diff(p[r]["values"], p[0]["values"]) for r in range(1, rounds)]
        new_vs_new = [_diff(q[r]["values"], q[0]["values"]) for r in range(1, rounds)]
        keys = list(p[0]["values"])
        floor = {k: max([d[k]["max_abs"] for d in parent_vs_parent] + [0.0]) for k in keys}
        worst = {k: max(d[k]["max_abs"] for d in new_vs_parent) for k in keys}
        values_ok = all(worst[k] <= floor[k] for k in keys)
        its = {s: [x["iterations"] for x in runs[s]] for s in sides}
        its_ok = len(set(its["parent"] + its["new"])) == 1
        pt = [t for x in p for t in x["times"]]
        nt = [t for x in q for t in x["times"]]
        time_ok = min(pt) <= statistics.median(nt) <= max(pt) or statistics.median(nt) <= statistics.median(pt)
        entry = {
            "rows": p[0]["rows"], "lanczos_rank": p[0]["rank"], "cg_iterations": its, "iterations_identical": its_ok,
            "bitwise_equal_to_parent": all(d[k]["bitwise"] for d in new_vs_parent for k in keys),
            "parent_reproduces_itself_bitwise": all(d[k]["bitwise"] for d in parent_vs_parent for k in keys),
            "max_abs_diff_new_vs_parent": worst, "max_abs_diff_parent_vs_parent": floor,
            "max_rel_diff_new_vs_parent": {k: max(d[k]["max_rel"] for d in new_vs_parent) for k in keys},
            "max_abs_diff_new_vs_new": {k: max([d[k]["max_abs"] for d in new_vs_new] + [0.0]) for k in keys},
            "values_within_parent_spread": values_ok,
            "inv_quad": {"parent": float(p[0]["values"]["inv_quad"].sum()), "new": float(q[0]["values"]["inv_quad"].sum())},
            "logdet": {"parent": float(p[0]["values"]["logdet"]), "new": float(q[0]["values"]["logdet"])},
            "mll_fwd_bwd_seconds": {"parent": {"median": statistics.median(pt), "min": min(pt), "max": max(pt)},
                                    "new": {"median": statistics.median(nt), "min": min(nt), "max": max(nt)}},
            "time_within_parent_spread": time_ok,
        }
        report["operators"][name] = entry
        ok = ok and values_ok and its_ok
        print(f"[{name}] rows {entry['rows']}: iterations {its}, bitwise {entry['bitwise_equal_to_parent']}, within parent spread {values_ok}, "
              f"time parent {entry['mll_fwd_bwd_seconds']['parent']['median'] * 1e3:.1f} ms new {entry['mll_fwd_bwd_seconds']['new']['median'] * 1e3:.1f} ms "
              f"(in spread: {time_ok})", flush=True)
        with open(out, "w") as fh:
            json.dump(report, fh, indent=1)
    report["ok"] = ok
    with open(out, "w") as fh:
        json.dump(report, fh, indent=1)
    print("ok" if ok else "DIFFERENT", "->", out)
    return 0 if ok else 1


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--export", nargs="?", const="HEAD", default=None, metavar="REV")
    ap.add_argument("--child", nargs=2, metavar=("OP", "FILE"))
    ap.add_argument("--ops", default=",".join(OPS))
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="time limit of one child process, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "added_diag_refactor_ab.json"))
    a = ap.parse_args()
    if a.export is not None:
        export(a.export)
        return 0
    if a.child:
        child(a.child[0], a.child[1], a.reps)
        return 0
    ops = [o for o in a.ops.split(",") if o]
    assert all(o in OPS for o in ops), ops
    return drive(ops, a.rounds, a.reps, os.path.abspath(a.out), a.limit)


if __name__ == "__main__":
    sys.exit(main())
