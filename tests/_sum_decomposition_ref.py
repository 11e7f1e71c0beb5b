"""numpy restatement of predict_mvn_sum / predict_sum (src/api.jl:898-1034) on top of oracle.infer_gp_sum and oracle.quantile, for
the tests of the batched sum-of-GPs entries.  Trees are the oracle's nested tuples (Node.to_tuple())."""
import numpy as np

from oracle import oracle as O


def predict_mvn_sum(splits, noises, ts, xs, ts_pred, y_transform=(1.0, 0.0), noise_pred=None):
    """Per particle (splits[k]: its component trees): raw-space (mean, cov) of Z = [F_1(T*); ...; F_M(T*); X(T*)] as
    predict_mvn_sum forms them — unapply_mean_var of the linear y_transform (slope a, intercept b), then + b / a on the F_1 rows —
    and the reference's indexes {"Y": slice, "F": [slices]}."""
    a, b = (float(v) for v in y_transform)
    comps, idx = [], None
    for trees, noise in zip(splits, noises):
        mu, S, iF, iX = O.infer_gp_sum(list(trees), float(noise), ts, xs, ts_pred, noise_pred=noise_pred)
        mr = (mu - b) / a
        mr[iF[0]] += b / a
        comps.append((mr, (1.0 / (a * a)) * S))
        idx = {"Y": iX, "F": iF}
    return comps, idx


def predict_sum(splits, noises, log_weights, ts, xs, ts_pred, y_transform=(1.0, 0.0), noise_pred=None, quantiles=()):
    """predict_sum's columns (ds, y_mean, component, particle, weight, y_<q>) in its row order: per particle, component 0 (Y), 1
    (F_1), 2 (F_2), each over ts_pred; quantiles by oracle.quantile on each component's raw marginals."""
    comps, idx = predict_mvn_sum(splits, noises, ts, xs, ts_pred, y_transform, noise_pred)
    w = O.particle_weights(np.asarray(log_weights, dtype=np.float64))
    p = len(ts_pred)
    cols = {"ds": [], "y_mean": [], "component": [], "particle": [], "weight": []}
    for q in quantiles:
        cols[f"y_{float(q)!r}"] = []
    for k, (mu, S) in enumerate(comps):
        X = O.quantile(mu, S, list(quantiles)) if len(quantiles) else None
        for c, blk in enumerate([idx["Y"]] + list(idx["F"])):
            cols["ds"].append(np.asarray(ts_pred, dtype=np.float64))
            cols["y_mean"].append(mu[blk])
            cols["component"].append(np.full(p, c))
            cols["particle"].append(np.full(p, k + 1))
            cols["weight"].append(np.full(p, w[k]))
            for j, q in enumerate(quantiles):
                cols[f"y_{float(q)!r}"].append(X[blk, j])
    return {k: np.concatenate(v) if v else np.zeros(0) for k, v in cols.items()}
