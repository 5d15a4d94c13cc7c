"""Parity checks shared by the CPU (host-simulation) and GPU (HIP) test files.

Every check drives the product engine (BatchedI2c -> C ABI -> kernels) and compares with
  (1) the golden vectors captured from the real reference (trajectory b = 0), and
  (2) the CPU oracle run on the same batched inputs.
Tolerances: the north star asks <= 1e-5 rel on means and <= 1e-4 rel on covariances for fp64;
the per-iteration checks below are far tighter (1e-9 ... 1e-7, max-norm relative).
"""
import importlib

import numpy as np
import torch

from golden_util import assert_close, assert_close_per_cell, elem_rtol_for, load_case, oracle_from_case

pkg = importlib.import_module("input-inference-for-control_amd")
from i2c.known_models import make_env_model  # noqa: E402  (the product's plugin registry)

FWD = ["mu_xu1_f", "sig_xu1_f", "mu_x3_f", "sig_x3_f", "J_dyn"]


def product_model(case):
    meta = case.meta
    m = make_env_model(meta["model"])
    if meta["model"] == "LinearKnown" and "noise" in meta:
        m.sig_x0 = meta["noise"] * np.eye(2)
        m.sig_eta = meta["noise"] * np.eye(2)
    if meta["model"] == "LinearKnown" and "goal" in meta:  # scripts/lqr_compare.py:128-131 on the product's plugin
        m.xag = meta["goal"] * np.ones((2, 1))
        m.zg_term = meta["goal"] * np.ones((2, 1))
        m.a = m.xag - m.A @ m.xag
    return m


def engine_from_case(case, lib, device, dtype=torch.float64, x0=None, mu_u=None, **kw):
    meta = case.meta
    eng = pkg.BatchedI2c(
        product_model(case), meta["T"], case.get("Q"), case["R"], case.get("Qf"), meta["alpha"], meta["tol"],
        case["mu_u"] if mu_u is None else mu_u, case["sig_u"], case.get("mu_x_term"), case.get("sig_x_term"),
        quad=tuple(kw.pop("quad", meta["quad"])), x0=x0, dtype=dtype, device=device, lib=lib, keep_prior=True,
        inference=meta.get("inference", "cubature"), gh_degree=meta.get("gh_degree"), **kw,
    )
    if meta.get("propagate"):
        eng._propagate = True
    if "use_expert_controller" in meta:
        eng.use_expert_controller = bool(meta["use_expert_controller"])
    if "tau" in meta:
        eng.tau = int(meta["tau"])
    return eng


def np_(t):
    return t.detach().to(torch.float64).cpu().numpy()


def close(a, b, tol, what):
    """Tight max-norm check at `tol` AND the element-wise check at the north star's numbers (1e-5 means, 1e-4 covariances / gains)."""
    assert_close(a, b, tol, what, elem_rtol=elem_rtol_for(what), atol_rel=max(1e-12, 0.01 * tol))


def compare_detail(eng, ref_get, it, tol, name, b=0, check_prop=False):
    """Compare every per-cell quantity of trajectory b with `ref_get(key)`: max-norm at `tol`, element-wise at the north star's
    tolerances, and the controller gain K cell by cell (each cell's own max-norm)."""
    f = eng.forward_messages()
    for k in FWD:
        close(np_(f[k])[b], ref_get(k), tol, f"{name} it{it} {k}")
    pmu, psig = eng.prior_state_action()
    close(np_(pmu)[b], ref_get("mu_xu0_f"), tol, f"{name} it{it} mu_xu0_f")
    close(np_(psig)[b], ref_get("sig_xu0_f"), tol, f"{name} it{it} sig_xu0_f")
    mu, sig = eng.marginal_state_action()
    close(np_(mu)[b], ref_get("mu_xu0_m"), tol, f"{name} it{it} mu_xu0_m")
    close(np_(sig)[b], ref_get("sig_xu0_m"), tol, f"{name} it{it} sig_xu0_m")
    K, k, sigK = eng.local_linear_policy()
    close(np_(K)[b], ref_get("K"), tol * 10, f"{name} it{it} K")
    assert_close_per_cell(np_(K)[b], ref_get("K"), 1e-4, f"{name} it{it} K")
    close(np_(k)[b], ref_get("k"), tol * 10, f"{name} it{it} k")
    close(np_(sigK)[b], ref_get("sigK"), tol * 10, f"{name} it{it} sigK")
    mz, sz = eng.observed_marginal()
    close(np_(mz)[b], ref_get("mu_z0_m"), tol, f"{name} it{it} mu_z0_m")
    close(np_(sz)[b], ref_get("sig_z0_m"), tol, f"{name} it{it} sig_z0_m")
    m3, s3 = eng.smoothed_next_state()
    close(np_(m3)[b], ref_get("mu_x3_m"), tol, f"{name} it{it} mu_x3_m")
    close(np_(s3)[b], ref_get("sig_x3_m"), tol, f"{name} it{it} sig_x3_m")
    if eng.has_Qf:
        mzt, szt = eng.terminal_observed_marginal()
        ref_m = ref_get("mu_z3_m")
        if ref_m is not None:
            close(np_(mzt)[b], ref_m, tol, f"{name} it{it} mu_z3_m")
            close(np_(szt)[b], ref_get("sig_z3_m"), tol, f"{name} it{it} sig_z3_m")
    if check_prop:
        p = eng.propagated()
        for key in ("mu_xu0_pf", "sig_xu0_pf", "mu_x3_pf", "sig_x3_pf"):
            close(np_(p[key])[b], ref_get(key), tol, f"{name} it{it} {key}")


def check_against_golden(name, lib, device, tol_detail=1e-8, tol_summary=1e-7, n_iters=None, dtype=torch.float64, **kw):
    """Free-running EM of the engine vs the reference's captured run (B = 1)."""
    g = load_case(name)
    eng = engine_from_case(g, lib, device, dtype=dtype, **kw)
    meta = g.meta
    if meta.get("calibrate_first"):
        eng.calibrate_alpha()
        assert_close(np_(eng.alpha)[0], g["alpha_calibrated"], tol_summary, "calibrated alpha")
    elif meta.get("propagate"):
        eng.propagate()
    detail = set(g.iters())
    n_total = len(g["costs_m"]) if n_iters is None else n_iters
    for it in range(1, n_total + 1):
        eng.em_iter += 1
        eng.forward_backward()
        if eng._propagate:
            eng.propagate()
        if it in detail:
            def ref_get(k, it=it):
                return g.at(it, k) if g.has(it, k) else None
            compare_detail(eng, ref_get, it, tol_detail, name, check_prop=eng._propagate)
        eng.maximize()
    assert eng.failures() == [], eng.failures()
    n = n_total
    H = eng.history
    assert_close(H(eng.alphas)[: n + 1, 0], g["alphas"][: n + 1], tol_summary, name + " alphas")
    assert_close(H(eng.alphas_desired)[: n + 1, 0], g["alphas_desired"][: n + 1], tol_summary, name + " alphas_desired")
    assert_close(H(eng.costs_m)[:n, 0], g["costs_m"][:n], tol_summary, name + " costs_m")
    assert_close(H(eng.costs_m_var)[:n, 0], g["costs_m_var"][:n], tol_summary, name + " costs_m_var")
    assert_close(H(eng.costs_pf)[:n, 0], g["costs_pf"][:n], tol_summary, name + " costs_pf")
    if "kl_terms" in g:
        assert_close(H(eng.kl_terms)[:n, 0], g["kl_terms"][:n], tol_summary * 100, name + " kl_terms")
    if "alphas_pf" in g:
        assert_close(H(eng.alphas_pf)[: n + 1, 0], g["alphas_pf"][: n + 1], tol_summary, name + " alphas_pf")
    if n == len(g["costs_m"]):
        K, k, sigK = eng.local_linear_policy()
        assert_close(np_(K)[0], g["final/K"], tol_summary * 10, name + " final K")
        assert_close(np_(k)[0], g["final/k"], tol_summary * 10, name + " final k")
        assert_close(np_(sigK)[0], g["final/sigK"], tol_summary * 10, name + " final sigK")
        mu, sig = eng.marginal_state_action()
        assert_close(np_(mu)[0], g["final/mu_xu0_m"], tol_summary, name + " final mu_xu0_m")
        assert_close(np_(sig)[0], g["final/sig_xu0_m"], tol_summary, name + " final sig_xu0_m")
    return eng


def batched_inputs(case, B, seed=1234, x0_scale=1e-2):
    """Deterministic per-trajectory variation: x0_b = x0 + 1e-2 eps_b, mu_u[b] from
    the legacy stream seeded with b; trajectory 0 is the unperturbed reference problem."""
    meta = case.meta
    x0 = case["x0"][None] + x0_scale * np.random.default_rng(seed).normal(size=(B, case["x0"].shape[0]))
    x0[0] = case["x0"]
    mu_u = np.empty((B, meta["T"], case["mu_u"].shape[1]))
    scale = float(np.abs(case["mu_u"]).max()) or 0.0
    for b in range(B):
        mu_u[b] = 1e-2 * np.random.RandomState(b).randn(*case["mu_u"].shape) if scale > 0 else 0.0
    mu_u[0] = case["mu_u"]
    return x0, mu_u


def with_horizon(case, T):
    """The same problem over T cells: meta["T"] replaced and the prior mean of the actions cut, or -- where T exceeds the golden's
    horizon -- tiled (it is only a prior mean)."""
    import json

    mu_u = case["mu_u"]
    mu_u = np.tile(mu_u, (-(-T // mu_u.shape[0]), 1))[:T]
    return type(case)({**dict(case), "meta": np.array(json.dumps({**case.meta, "T": int(T)})), "mu_u": mu_u})


def check_batch_against_oracle(name, lib, device, B, n_iters, tol=1e-8, dtype=torch.float64, tol_policy=None, T=None,
                               optional_outputs=False, **kw):
    """Batched engine vs the batched CPU oracle on identical inputs, all trajectories, every cell. T: another horizon than the
    golden case's (with_horizon). optional_outputs: the engine also writes the smoothed state entering every cell, the observed
    marginal and the per-cell cost statistics (the walkers' non-lean variants), and those are compared too."""
    g = load_case(name)
    if T is not None:
        g = with_horizon(g, T)
    meta_override = kw.pop("meta_override", None)
    if meta_override:  # the same case with other hyper-parameters (e.g. the temperature), for the engine AND the oracle
        import json

        g = type(g)({**dict(g), "meta": np.array(json.dumps({**g.meta, **meta_override}))})
    x0, mu_u = batched_inputs(g, B)
    if optional_outputs:
        kw = dict(kw, keep_xm=True, keep_zpost=True)
    eng = engine_from_case(g, lib, device, dtype=dtype, x0=x0, mu_u=mu_u, **kw)
    if optional_outputs:
        eng.cell_stats = torch.zeros(eng.H, 2, eng.B, dtype=eng.dtype, device=eng.device)
    g2 = dict(g)
    if "quad" in kw:  # the cubature weights asked of the engine: the oracle integrates with the same rule
        import json

        g2["meta"] = np.array(json.dumps({**g.meta, "quad": list(kw["quad"])}))
    o = oracle_from_case(type(g)({**g2, "mu_u": mu_u}), x0=x0)
    if g.meta.get("propagate"):
        eng.propagate()
        o.propagate()
    tol_policy = tol * 10 if tol_policy is None else tol_policy
    for it in range(1, n_iters + 1):
        eng.learn_msgs()
        o.learn_msgs()
        f = eng.forward_messages()
        for k in FWD:
            close(np_(f[k]), getattr(o, k), tol, f"{name} B={B} it{it} {k}")
        mu, sig = eng.marginal_state_action()
        close(np_(mu), o.mu_xu0_m, tol, f"{name} B={B} it{it} mu_xu0_m")
        close(np_(sig), o.sig_xu0_m, tol, f"{name} B={B} it{it} sig_xu0_m")
        K, k, sigK = eng.local_linear_policy()
        close(np_(K), o.K, tol_policy, f"{name} B={B} it{it} K")
        Kc = np_(K)  # every (b, t) cell of the gain on its own
        assert_close_per_cell(Kc.reshape((-1,) + Kc.shape[2:]), np.asarray(o.K).reshape((-1,) + Kc.shape[2:]), 1e-4, f"{name} B={B} it{it} K")
        close(np_(k), o.k, tol_policy, f"{name} B={B} it{it} k")
        close(np_(sigK), o.sigK, tol_policy, f"{name} B={B} it{it} sigK")
        close(np_(eng.alpha), o.alpha, tol, f"{name} B={B} it{it} alpha")
        close(np_(eng.costs_m[-1]), o.costs_m[-1], tol, f"{name} B={B} it{it} cost")
        if optional_outputs:
            m3, s3 = eng.smoothed_next_state()
            close(np_(m3), o.mu_x3_m, tol, f"{name} B={B} it{it} mu_x3_m")
            close(np_(s3), o.sig_x3_m, tol, f"{name} B={B} it{it} sig_x3_m")
            mz, sz = eng.observed_marginal()
            close(np_(mz), o.mu_z0_m, tol, f"{name} B={B} it{it} mu_z0_m")
            close(np_(sz), o.sig_z0_m, tol, f"{name} B={B} it{it} sig_z0_m")
            cm, cv = o._gaussian_cost(o.mu_z0_m, o.sig_z0_m)  # (B, T): the cost mean and variance of every cell
            close(np_(eng.cell_stats[:, 0]).T, cm, tol, f"{name} B={B} it{it} cell cost")
            close(np_(eng.cell_stats[:, 1]).T, cv, tol, f"{name} B={B} it{it} cell cost variance")
    assert eng.failures() == []
    return eng, o
