"""SPEC §23.3: a Fourier-basis initiation classifier fitted by IRLS — logistic regression on the basis of order p, a Newton iteration
whose Hessian is the weighted feature Gram and whose gradient is the unweighted moment of the same samples (ScgContext.
basis_gram_irls, on the terms of ScgContext.logistic_terms). Host code, float64; the hot parts are those two calls and
ScgContext.basis_values. A reporting instrument (SPEC §18's sense): nothing acts or learns with such a classifier.
SPEC §24.3, at the end: the parts of SkillChainingAgent.improve_initiation — §6's quadratic refitted on trial labels
(refit_quadratic), the candidate classifier tables (candidate_tables) and §21.4's rule over them (choose_table)."""
from typing import Optional

import numpy as np
import torch

from . import _lib
from .core import fourier_scale_table

MASKS = ("state", "position")
# SPEC §23.3: ten times the largest floor of ||g||inf / ||g at w = 0||inf the binary32 path reached on the three test problems
# (profiles/r29_irls_fit_floor.txt)
DEFAULT_TOL = 1.5e-4
MAX_HALVINGS = 30


def feature_mask(order: int, kind: str = "state") -> np.ndarray:
    """bool [F]: "state" every feature of order `order`, "position" the (p + 1)^2 features with c3 = c4 = 0 (no velocity)."""
    F = _lib.basis_features(order)
    if kind not in MASKS:
        raise ValueError(f"the feature mask must be one of {MASKS}")
    if kind == "state":
        return np.ones(F, bool)
    return np.arange(F) % (order + 1) ** 2 == 0


def penalty(order: int, ridge: float) -> np.ndarray:
    """lambda float64 [F] = ridge / scale_f^2 (SPEC §16.3's Lambda over n) with lambda_0 = 0: the constant feature is free."""
    lam = float(ridge) / fourier_scale_table(order).astype(np.float64) ** 2
    lam[0] = 0.0
    return lam


def penalised_loss(z, label, w, lam) -> float:
    """L(w) = mean_n [log(1 + exp(z_n)) - l_n z_n] + 1/2 sum_f lambda_f w_f^2, in float64 from the logits given."""
    z = np.asarray(z).astype(np.float64)
    l = np.asarray(label) != 0
    w = np.asarray(w, np.float64)
    return float(np.mean(np.logaddexp(0.0, z) - np.where(l, z, 0.0)) + 0.5 * np.sum(np.asarray(lam, np.float64) * w * w))


class DeviceGram:
    """The device half of one IRLS iteration on a fixed sample set: `values(w)` = scg_basis_values of w as binary32, and
    `hessian_gradient(z)` = (H, grad) of scg_basis_gram_irls on scg_logistic_terms(z, label). irls_fit's `gram=` takes any object
    with these two methods (a host test's numpy model)."""

    def __init__(self, ctx, order: int, s, label):
        self.ctx, self.order = ctx, int(order)
        self.s = [torch.as_tensor(v, dtype=torch.float32).to(ctx.device).contiguous().view(-1) for v in s]
        self.n = self.s[0].numel()
        self.label = (torch.as_tensor(label).to(ctx.device).view(-1) != 0).to(torch.uint8).contiguous()

    def values(self, w) -> np.ndarray:
        V = torch.from_numpy(np.asarray(w, np.float64).astype(np.float32)[None, :].copy()).to(self.ctx.device)
        return self.ctx.basis_values(self.order, self.s, V)[0].cpu().numpy()

    def hessian_gradient(self, z):
        zd = torch.from_numpy(np.ascontiguousarray(z, np.float32)).to(self.ctx.device)
        _, rw, e = self.ctx.logistic_terms(zd, self.label)
        H, grad = self.ctx.basis_gram_irls(self.order, self.s, [0, self.n], rw, e)
        return H[0].cpu().numpy().astype(np.float64), grad[0].cpu().numpy().astype(np.float64)


def irls_fit(ctx, order: int, s, label, mask: str = "state", ridge: float = 1e-3, tol: float = DEFAULT_TOL, max_iter: int = 25,
             w0=None, gram=None):
    """Fit w [F] (float64; exactly +0 outside `mask`) to the labels by SPEC §23.3's damped Newton iteration. Returns (w, history,
    reason): history one dict per evaluated iterate (L, g = ||g||inf over the mask, and for the step taken from it t and
    halvings), reason one of "tol", "no halving lowers L", "max_iter". ValueError for a one-class label set."""
    lab = np.asarray(label.cpu() if isinstance(label, torch.Tensor) else label).reshape(-1) != 0
    n = lab.size
    if n == 0 or lab.all() or not lab.any():
        raise ValueError("irls_fit: the labels hold one class only (with a free intercept the optimum is at infinity)")
    F = _lib.basis_features(order)
    idx = np.flatnonzero(feature_mask(order, mask))
    lam = penalty(order, ridge)
    gram = DeviceGram(ctx, order, s, lab) if gram is None else gram

    def evaluate(w):
        z = gram.values(w)
        return z, penalised_loss(z, lab, w, lam)

    def newton_terms(w, z):
        H, grad = gram.hessian_gradient(z)
        g = grad[idx] / n - lam[idx] * w[idx]
        M = H[np.ix_(idx, idx)] / n + np.diag(lam[idx])
        return g, M

    w = np.zeros(F, np.float64)
    z, L = evaluate(w)
    g, M = newton_terms(w, z)
    g0 = float(np.max(np.abs(g)))
    if w0 is not None:
        w[idx] = np.asarray(w0, np.float64).reshape(F)[idx]
        z, L = evaluate(w)
        g, M = newton_terms(w, z)
    history, reason = [], "max_iter"
    for it in range(int(max_iter) + 1):
        gn = float(np.max(np.abs(g)))
        history.append({"L": L, "g": gn, "t": None, "halvings": None})
        if gn <= tol * g0:
            reason = "tol"
            break
        if it == max_iter:
            break
        Lc = np.linalg.cholesky(np.tril(M) + np.tril(M, -1).T)              # (the lower triangle is read, as ridge_solve reads it)
        d = np.linalg.solve(Lc.T, np.linalg.solve(Lc, g))
        t, taken = 1.0, None
        for h in range(MAX_HALVINGS + 1):
            cand = w.copy()
            cand[idx] = w[idx] + t * d
            zc, Lcand = evaluate(cand)
            if Lcand < L:
                taken = (cand, zc, Lcand, t, h)
                break
            t *= 0.5
        if taken is None:
            reason = "no halving lowers L"
            break
        w, z, L = taken[0], taken[1], taken[2]
        history[-1].update(t=taken[3], halvings=taken[4])
        g, M = newton_terms(w, z)
    return w, history, reason


class FourierClassifier:
    """sign(w . phi(s)) on the basis of order `order`: in the set where the logit is positive. `mask` names the features the fit
    was given ("state" or "position"); the weights outside it are +0."""

    def __init__(self, order: int, mask: str, w):
        F = _lib.basis_features(order)
        self.order, self.mask = int(order), str(mask)
        self.w = np.asarray(w, np.float64).reshape(F).copy()
        if np.any(self.w[~feature_mask(order, mask)] != 0):
            raise ValueError("FourierClassifier: a weight outside the feature mask is not zero")

    def logits(self, ctx, s) -> torch.Tensor:
        """z float32 [n] on ctx's device: scg_basis_values of the weights as binary32 (SPEC §18.3's order)."""
        st = [torch.as_tensor(v, dtype=torch.float32).to(ctx.device).contiguous().view(-1) for v in s]
        V = torch.from_numpy(self.w.astype(np.float32)[None, :].copy()).to(ctx.device)
        return ctx.basis_values(self.order, st, V)[0]

    def predict(self, ctx, s) -> torch.Tensor:
        """uint8 [n]: z > 0."""
        return (self.logits(ctx, s) > 0).to(torch.uint8)

    def state_dict(self) -> dict:
        return {"order": self.order, "mask": self.mask, "w": self.w.copy()}


def classification_stats(pred, outcome, z=None) -> dict:
    """tp / fp / fn / tn of `pred` (predicted in the set) against `outcome` (the trial succeeded), precision, recall (NaN when
    their denominator is empty), accuracy and, with the logits `z`, the mean log-loss (NaN without)."""
    p, s = np.asarray(pred).reshape(-1) != 0, np.asarray(outcome).reshape(-1) != 0
    tp, fp, fn, tn = (int(v) for v in (np.sum(p & s), np.sum(p & ~s), np.sum(~p & s), np.sum(~p & ~s)))
    nan = float("nan")
    n = tp + fp + fn + tn
    out = {"tp": tp, "fp": fp, "fn": fn, "tn": tn,
           "precision": tp / (tp + fp) if tp + fp else nan,
           "recall": tp / (tp + fn) if tp + fn else nan,
           "accuracy": (tp + tn) / n if n else nan,
           "log_loss": nan}
    if z is not None and n:
        z = np.asarray(z).astype(np.float64).reshape(-1)
        out["log_loss"] = float(np.mean(np.logaddexp(0.0, z) - np.where(s, z, 0.0)))
    return out


# ---------------------------------------------------------------------------------------------------- SPEC §24.3: the safeguarded refit step

def refit_quadratic(ctx, w8, xy, label, iters: int = 400, lr: float = 3.0, l2: float = 1e-4) -> torch.Tensor:
    """SPEC §6's fit (scg_fit_initiation) of ONE row, started from a copy of `w8`, on the examples xy [M][2] with `label` [M]
    (non-zero: positive), on `ctx`. Returns the new row (float32 [8] on ctx's device); `w8` itself is never written."""
    w = torch.as_tensor(w8, dtype=torch.float32).to(ctx.device).reshape(-1).clone().contiguous()
    xy = torch.as_tensor(xy, dtype=torch.float32).to(ctx.device).contiguous().view(-1)
    lab = (torch.as_tensor(label).to(ctx.device).view(-1) != 0).to(torch.uint8).contiguous()
    off = torch.tensor([0, lab.numel()], dtype=torch.int32, device=ctx.device)
    ctx.fit_initiation(xy, lab, off, w, iters, lr, l2)
    return w


def candidate_tables(clf, rows: dict) -> list:
    """The candidate classifier tables of improve_initiation, a pure function: `clf` the shipped table [n_vf][8], `rows` {k: w8} the
    refitted rows. Returns [(label, table)]: "shipped" first (a copy of clf), then "k" for each fitted k, ascending, with row k alone
    replaced, then "all" (every fitted row replaced) when two or more rows were fitted. Neither input is written."""
    clf = torch.as_tensor(clf)
    ks = sorted(int(k) for k in rows)
    if any(not (0 <= k < clf.shape[0]) for k in ks):
        raise ValueError(f"candidate_tables: a fitted row is outside the table's {clf.shape[0]} rows")

    def with_rows(which):
        t = clf.clone()
        for k in which:
            t[k] = torch.as_tensor(rows[k], dtype=clf.dtype).to(clf.device).reshape(clf.shape[1:])
        return t

    out = [("shipped", with_rows(()))] + [(str(k), with_rows((k,))) for k in ks]
    if len(ks) >= 2:
        out.append(("all", with_rows(ks)))
    return out


def choose_table(candidates, criterion: str = "discounted", z: float = 2.0) -> dict:
    """SPEC §21.4's rule over labelled candidates [{"label", "summary", "paired"}], "shipped" first and `paired` against it: the
    candidate with the highest mean of `criterion`, ties to the earlier, a NaN mean never; accepted only where its paired mean
    difference against "shipped" exceeds z standard errors (se = 0: where it exceeds 0). valuefit.choose_candidate decides: a
    candidate's position stands in for its lambda, so "shipped" (position 0) is the table that is kept. Returns {"index", "label"
    (of the pick; None when every mean is a NaN), "chosen" ("shipped" unless accepted), "accepted"}."""
    from .valuefit import choose_candidate
    cands = list(candidates)
    if not cands or cands[0]["label"] != "shipped":
        raise ValueError("choose_table: the first candidate must be 'shipped'")
    pick = choose_candidate([{"lambda": float(i), "summary": c["summary"], "paired": c["paired"]} for i, c in enumerate(cands)],
                            criterion, z)
    label = None if pick["index"] is None else cands[pick["index"]]["label"]
    return {"index": pick["index"], "label": label, "chosen": label if pick["accepted"] else "shipped", "accepted": pick["accepted"]}
