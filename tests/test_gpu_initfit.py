"""initfit.irls_fit on the device (SPEC §23.3) against the float64 reference — materialised scg_basis_features and the host IRLS of
tests/irls_gram_model.py — on the problems (a) and (c) of tests/test_initfit_host.py at order 3: the penalised loss at the device's
weights is within MARGIN of the reference's minimum (the reference is a minimum, so the difference is second order in the weight
error), L never rises, masked weights are exactly +0; (c)'s two held-out accuracies; and SkillChainingAgent.fit_initiation_fourier on
the rig's small agent: the report's counts add up, initiation_report without classifier= keeps its bits, training is left alone.

Measured on the MI355X at the default tol (profiles/r29_irls_fit_floor.txt): (L(w_gpu) - L(w_ref)) / |L(w_ref)| was 8.6e-09
(bernoulli, state), 1.0e-10 (bernoulli, position), 2.4e-06 (vx, state) and 1.4e-15 (vx, position); MARGIN is ten times the largest."""
import numpy as np
import pytest
import torch

import irls_gram_model as IM
import skill_chaining_with_graphs_amd as scg
from skill_chaining_with_graphs_amd import _lib, initfit
from skill_chaining_with_graphs_amd.core import ScgContext
from gpu_util import dev, gestating_agent, spy_calls
from util import HP, make_oracle

pytestmark = pytest.mark.gpu

ORDER, N = 3, 4096
MARGIN = 2.4e-5               # ten times the largest relative difference measured (above)


@pytest.fixture(scope="module")
def rig():
    _, m = make_oracle("pinball_simple")
    ctx = ScgContext(64, 0, m, device=0, block_envs=256, **HP)
    out = {}
    for name in ("bernoulli", "vx"):
        s, lab = IM.problem(name, N)
        phi = ctx.basis_features(ORDER, [dev(v) for v in s]).cpu().numpy().astype(np.float64)
        out[name] = dict(s=s, lab=lab, phi=phi)
    yield ctx, out
    ctx.close()


def both_fits(ctx, p, mask, rows=slice(None)):
    s, lab, phi = [v[rows] for v in p["s"]], p["lab"][rows], p["phi"][rows]
    w_ref, h_ref, r_ref = initfit.irls_fit(None, ORDER, None, lab, mask=mask, tol=1e-9, gram=IM.Float64Gram(phi, lab))
    w, hist, reason = initfit.irls_fit(ctx, ORDER, s, lab, mask=mask)
    lam = initfit.penalty(ORDER, 1e-3)
    L = lambda v: initfit.penalised_loss(phi @ v, lab, v, lam)
    return w, hist, reason, w_ref, r_ref, L(w), L(w_ref)


@pytest.mark.parametrize("name,mask", [("bernoulli", "state"), ("bernoulli", "position"), ("vx", "state"), ("vx", "position")])
def test_device_fit_reaches_the_float64_minimum(rig, name, mask):
    ctx, problems = rig
    w, hist, reason, w_ref, r_ref, L_gpu, L_ref = both_fits(ctx, problems[name], mask)
    Ls = [h["L"] for h in hist]
    print(f"{name} {mask}: {len(hist) - 1} iterations, {reason}; g / g0 {hist[-1]['g'] / hist[0]['g']:.3e}; L_gpu {L_gpu:.15f} L_ref {L_ref:.15f} "
          f"(L_gpu - L_ref) / |L_ref| {(L_gpu - L_ref) / abs(L_ref):.3e}; max |w - w_ref| {np.max(np.abs(w - w_ref)):.3e}")
    assert r_ref == "tol"
    assert all(b <= a for a, b in zip(Ls, Ls[1:])), Ls
    assert reason == "tol" and len(hist) - 1 <= 25
    assert L_gpu - L_ref <= MARGIN * abs(L_ref)
    m = initfit.feature_mask(ORDER, mask)
    assert w.dtype == np.float64 and not w[~m].view(np.uint64).any()


def test_velocity_labels_need_velocity_features_on_the_device(rig):
    ctx, problems = rig
    p = problems["vx"]
    held = slice(1, None, 2)
    sd = [dev(v[held]) for v in p["s"]]
    acc = {}
    for mask in ("position", "state"):
        w, hist, reason = initfit.irls_fit(ctx, ORDER, [v[0::2] for v in p["s"]], p["lab"][0::2], mask=mask)
        clf = initfit.FourierClassifier(ORDER, mask, w)
        z = clf.logits(ctx, sd)
        pred = clf.predict(ctx, sd)
        assert torch.equal(pred, (z > 0).to(torch.uint8)) and pred.dtype == torch.uint8
        st = initfit.classification_stats(pred.cpu().numpy(), p["lab"][held], z.cpu().numpy())
        acc[mask] = st["accuracy"]
        print(f"vx > 0, {mask}: held-out accuracy {st['accuracy']:.4f}, log-loss {st['log_loss']:.4f}, {len(hist) - 1} iterations, {reason}")
    assert acc["position"] <= 0.6 and acc["state"] >= 0.95


def test_one_class_is_refused_before_any_launch(rig):
    ctx, problems = rig
    with spy_calls(ctx) as (calls, _):
        with pytest.raises(ValueError, match="one class"):
            initfit.irls_fit(ctx, ORDER, problems["vx"]["s"], np.ones(N, bool))
    assert calls == []


def near_target_states(m, n, seed):
    """Start states around option 1's target (the goal): inside it and up to four radii out, with velocities: both outcomes occur."""
    rng = np.random.default_rng(seed)
    tx, ty, r = m.target
    rad, ang = rng.uniform(0, 4 * r, n), rng.uniform(0, 2 * np.pi, n)
    x, y = np.clip(tx + rad * np.cos(ang), 0.02, 0.98), np.clip(ty + rad * np.sin(ang), 0.02, 0.98)
    return [v.astype(np.float32) for v in (x, y, rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n))]


def test_fit_initiation_fourier_reports_and_leaves_training_alone():
    a, b = gestating_agent(n=512), gestating_agent(n=512)
    states = near_target_states(a.map, 512, 5)
    calls = []
    out = {}

    def probe():
        with spy_calls(a.ctx, calls):
            out["plain"] = a.initiation_report(1, states)
            out["fit"] = a.fit_initiation_fourier(1, states, order=3, features="state")
            out["reuse"] = a.fit_initiation_fourier(1, order=3, features="position", trials=out["fit"][1])
            out["with"] = a.initiation_report(1, states, classifier=out["fit"][0])

    for i in range(6):
        if i == 2:
            W0, clf0 = a.W.clone(), a.clf.clone()
            probe()
            assert torch.equal(a.W, W0) and torch.equal(a.clf, clf0)
        a.step_batch()
        b.step_batch()
    torch.cuda.synchronize()
    assert calls == [], f"the fit called into the training context: {calls}"
    assert torch.equal(a.W, b.W) and torch.equal(a.clf, b.clf) and a.t == b.t == 6
    for f in scg.EnvState.FIELDS:
        assert torch.equal(getattr(a.state, f), getattr(b.state, f)), f

    plain, (clf, rep), (clf2, rep2), with_clf = out["plain"], out["fit"], out["reuse"], out["with"]
    # the default report: the parent's numbers, recounted by hand from in_k and the outcomes
    pred = a._trial_ctx.classifier_predict(plain["states"][0], plain["states"][1], clf0[1].contiguous()).cpu().numpy().astype(bool)
    s = plain["trials"].outcome.cpu().numpy() == _lib.TRIAL_SUCCESS
    tp, fp, fn, tn = (int(v) for v in (np.sum(pred & s), np.sum(pred & ~s), np.sum(~pred & s), np.sum(~pred & ~s)))
    assert (plain["tp"], plain["fp"], plain["fn"], plain["tn"]) == (tp, fp, fn, tn) and plain["n"] == 512
    nan = float("nan")
    for key, want in (("precision", tp / (tp + fp) if tp + fp else nan), ("recall", tp / (tp + fn) if tp + fn else nan),
                      ("success_in", tp / (tp + fp) if tp + fp else nan), ("success_out", fn / (fn + tn) if fn + tn else nan)):
        assert np.array_equal(np.float64(plain[key]).view(np.uint64), np.float64(want).view(np.uint64)), key
    assert np.array_equal(plain["predicted"].cpu().numpy().astype(bool), pred) and plain["predicted"].dtype == torch.uint8
    assert 0 < s.sum() < 512
    # the fit's report: the halves are the even- and the odd-indexed states, the counts add up, the shipped half is in_k's
    assert rep["fit"]["n"] == rep["held_out"]["n"] == 256 and rep["n"] == 512 and rep["order"] == 3 and rep["features"] == "state"
    assert torch.equal(rep["trials"].outcome, plain["trials"].outcome)
    for half, rows in (("fit", slice(0, None, 2)), ("held_out", slice(1, None, 2))):
        for who in ("fourier", "shipped"):
            st = rep[half][who]
            assert st["tp"] + st["fp"] + st["fn"] + st["tn"] == 256
            assert st["tp"] + st["fn"] == int(s[rows].sum())
        assert rep[half]["shipped"]["tp"] == int(np.sum(pred[rows] & s[rows]))
        assert np.isfinite(rep[half]["fourier"]["log_loss"]) and np.isnan(rep[half]["shipped"]["log_loss"])
    assert rep["reason"] in ("tol", "no halving lowers L", "max_iter") and rep["iterations"] == len(rep["history"]) - 1
    Ls = [h["L"] for h in rep["history"]]
    assert all(y <= x for x, y in zip(Ls, Ls[1:]))
    assert rep["fit"]["fourier"]["accuracy"] >= rep["fit"]["shipped"]["accuracy"] - 0.05      # 256 weights on 256 labels fit them
    print({h: {w: round(rep[h][w]["accuracy"], 4) for w in ("fourier", "shipped")} for h in ("fit", "held_out")}, rep["reason"])
    # trials= reuses the states and outcomes: no new trial, the same labels
    assert rep2["trials"] is rep["trials"] and rep2["features"] == "position"
    assert not clf2.w[~initfit.feature_mask(3, "position")].any()
    # initiation_report(classifier=): predicted comes from the classifier, the trials are the same
    want = clf.predict(a._trial_ctx, with_clf["states"])
    assert torch.equal(with_clf["predicted"], want) and torch.equal(with_clf["predicted"], rep["predicted"])
    assert torch.equal(with_clf["trials"].outcome, plain["trials"].outcome)
    assert with_clf["tp"] + with_clf["fp"] + with_clf["fn"] + with_clf["tn"] == 512
    assert with_clf["tp"] == rep["fit"]["fourier"]["tp"] + rep["held_out"]["fourier"]["tp"]
