"""SPEC §23.3 on the host (no GPU): initfit.irls_fit with a numpy model in the place of the device calls (irls_gram_model.
Float64Gram on basis_model's order-3 features) on the three test problems — Bernoulli labels from a known row, a disc in position
under two ridges, labels vx > 0 —: L never rises, the fit stops on its tolerance within 25 iterations at tol = 1e-9, masked weights
are exactly +0, a one-class set is refused; and on vx > 0 a position classifier cannot learn what a state classifier can."""
import numpy as np
import pytest

import basis_model as BM
import irls_gram_model as IM

ORDER, N = 3, 4096


@pytest.fixture(scope="module")
def problems(pkg):
    out = {}
    for name in ("bernoulli", "disc", "vx"):
        s, lab = IM.problem(name, N)
        out[name] = dict(s=s, lab=lab, phi=BM.features(ORDER, *s).astype(np.float64))
    return out


def fit(problems, name, mask, ridge=1e-3, half=None, **kw):
    from skill_chaining_with_graphs_amd import initfit
    p = problems[name]
    rows = slice(None) if half is None else slice(half, None, 2)
    gram = IM.Float64Gram(p["phi"][rows], p["lab"][rows])
    return initfit.irls_fit(None, ORDER, None, p["lab"][rows], mask=mask, ridge=ridge, tol=1e-9, gram=gram, **kw)


CASES = [("bernoulli", "state", 1e-3), ("bernoulli", "position", 1e-3), ("disc", "position", 1e-3), ("disc", "position", 1e-5),
         ("disc", "state", 1e-3), ("vx", "state", 1e-3), ("vx", "position", 1e-3)]


@pytest.mark.parametrize("name,mask,ridge", CASES)
def test_fit_descends_and_stops_on_its_tolerance(problems, name, mask, ridge):
    from skill_chaining_with_graphs_amd import initfit
    w, hist, reason = fit(problems, name, mask, ridge)
    L = [h["L"] for h in hist]
    print(f"{name} {mask} ridge {ridge}: {len(hist) - 1} iterations, {reason}, L {L[0]:.6f} -> {L[-1]:.6f}, g {hist[-1]['g']:.3e}")
    assert all(b <= a for a, b in zip(L, L[1:])), L                    # L never rises
    assert reason == "tol" and len(hist) - 1 <= 25
    assert hist[-1]["g"] <= 1e-9 * hist[0]["g"] and L[0] == pytest.approx(np.log(2.0), abs=1e-12)
    assert all(h["t"] is not None and 0 <= h["halvings"] <= 30 for h in hist[:-1]) and hist[-1]["t"] is None
    m = initfit.feature_mask(ORDER, mask)
    assert w.dtype == np.float64 and w.shape == (256,)
    assert not w[~m].view(np.uint64).any()                             # exactly +0 outside the mask
    assert np.count_nonzero(w[m]) == m.sum()
    # the stopping point is the penalised optimum: the float64 gradient of L vanishes there
    p = problems[name]
    z = p["phi"] @ w
    g = p["phi"].T @ ((p["lab"] != 0) - 1.0 / (1.0 + np.exp(-z))) / N - initfit.penalty(ORDER, ridge) * w
    assert np.max(np.abs(g[m])) <= 1e-9 * hist[0]["g"] * 1.0001


def test_feature_masks_and_penalty(pkg):
    from skill_chaining_with_graphs_amd import initfit
    for order in (3, 5, 7):
        c = BM.coefficients(order)
        pos = initfit.feature_mask(order, "position")
        assert pos.sum() == (order + 1) ** 2 and np.array_equal(pos, (c[:, 2] == 0) & (c[:, 3] == 0))
        assert initfit.feature_mask(order, "state").all()
        lam = initfit.penalty(order, 1e-3)
        assert lam[0] == 0 and np.allclose(lam[1:], 1e-3 * (c[1:] ** 2).sum(1), rtol=1e-6)
    with pytest.raises(ValueError):
        initfit.feature_mask(3, "velocity")
    with pytest.raises(pkg.ScgError):
        initfit.feature_mask(4, "state")


def test_a_one_class_set_is_refused(problems):
    from skill_chaining_with_graphs_amd import initfit
    p = problems["disc"]
    for lab in (np.zeros(N, bool), np.ones(N, np.uint8), np.zeros(0, bool)):
        with pytest.raises(ValueError, match="one class"):
            initfit.irls_fit(None, ORDER, None, lab, gram=IM.Float64Gram(p["phi"][:len(lab)], lab))


def test_a_warm_start_stops_at_once_and_max_iter_is_kept(problems):
    w, hist, reason = fit(problems, "bernoulli", "state")
    w2, hist2, reason2 = fit(problems, "bernoulli", "state", w0=w)
    assert reason2 == "tol" and len(hist2) == 1 and np.array_equal(w2, w)
    w3, hist3, reason3 = fit(problems, "bernoulli", "state", max_iter=2)
    assert reason3 == "max_iter" and len(hist3) == 3 and hist3[-1]["L"] < hist3[0]["L"]


def test_velocity_labels_need_velocity_features(problems):
    """(c): labels vx > 0. Fitted on the even-indexed states, judged on the odd-indexed ones: a classifier of position is at
    chance (<= 0.6), one of the full state learns the edge (>= 0.95)."""
    from skill_chaining_with_graphs_amd import initfit
    p = problems["vx"]
    acc = {}
    for mask in ("position", "state"):
        w, hist, reason = fit(problems, "vx", mask, half=0)
        held = slice(1, None, 2)
        z = p["phi"][held] @ w
        st = initfit.classification_stats(z > 0, p["lab"][held], z)
        assert st["tp"] + st["fp"] + st["fn"] + st["tn"] == N // 2
        acc[mask] = st["accuracy"]
        print(f"vx > 0, {mask}: held-out accuracy {st['accuracy']:.4f}, log-loss {st['log_loss']:.4f}, {len(hist) - 1} iterations")
    assert acc["position"] <= 0.6 and acc["state"] >= 0.95


def test_classification_stats(pkg):
    from skill_chaining_with_graphs_amd import initfit
    st = initfit.classification_stats([1, 1, 0, 0, 1], [1, 0, 0, 1, 1], z=[2.0, 1.0, -1.0, -3.0, 0.5])
    assert (st["tp"], st["fp"], st["fn"], st["tn"]) == (2, 1, 1, 1)
    assert st["precision"] == 2 / 3 and st["recall"] == 2 / 3 and st["accuracy"] == 3 / 5
    ll = np.mean([np.log1p(np.exp(-2.0)), np.log1p(np.exp(1.0)), np.log1p(np.exp(-1.0)), np.log1p(np.exp(3.0)), np.log1p(np.exp(-0.5))])
    assert st["log_loss"] == pytest.approx(ll, rel=1e-12)
    empty = initfit.classification_stats([0, 0], [0, 0])
    assert np.isnan(empty["precision"]) and np.isnan(empty["recall"]) and empty["accuracy"] == 1.0 and np.isnan(empty["log_loss"])
    c = initfit.FourierClassifier(3, "position", np.zeros(256))
    assert c.state_dict()["order"] == 3 and c.state_dict()["mask"] == "position"
    bad = np.zeros(256)
    bad[1] = 1.0                                                       # a velocity weight under the position mask
    with pytest.raises(ValueError):
        initfit.FourierClassifier(3, "position", bad)
