"""Anomaly scoring after AnoGAN (Schlegl et al. 2017), host side: the score that Sampler.anomaly's projection ends in, and the
rank-based AUROC of scores against known flags.  The projection itself - the residual and the feature-matching term on the
discriminator's activations - is DcganEngine.project(feature_target=...)."""
import torch

from ._lib import JckError


def anomaly_score(residual, feature, lam):
    """(1 - lam) * residual + lam * feature in fp64, lam in [0, 1): AnoGAN's A(x) = (1 - lambda) R(x) + lambda D(x)."""
    lam = float(lam)
    if not 0.0 <= lam < 1.0:
        raise JckError(f"anomaly_score: lam must lie in [0, 1), got {lam}")
    r, f = torch.as_tensor(residual).to(torch.float64), torch.as_tensor(feature).to(torch.float64)
    if r.shape != f.shape:
        raise JckError(f"anomaly_score: residual {tuple(r.shape)} and feature {tuple(f.shape)} differ in shape")
    return (1.0 - lam) * r + lam * f


def auroc(scores, anomalous):
    """The area under the ROC curve of `scores` [n] as a detector of `anomalous` [n] (bool): the Mann-Whitney estimate, the share of
    (anomalous, normal) pairs that the scores order correctly, ties counting half, in fp64.  JckError when a class is empty or a
    score is NaN."""
    s = torch.as_tensor(scores).detach().to("cpu", torch.float64).view(-1)
    a = torch.as_tensor(anomalous).detach().to("cpu").view(-1)
    if a.dtype != torch.bool:
        if bool(((a != 0) & (a != 1)).any()):
            raise JckError("auroc: anomalous must be bool (or 0 / 1)")
        a = a != 0
    if s.numel() != a.numel():
        raise JckError(f"auroc: {s.numel()} scores for {a.numel()} flags")
    if bool(torch.isnan(s).any()):
        raise JckError("auroc: a score is NaN")
    pos, neg = s[a], s[~a]
    if pos.numel() == 0 or neg.numel() == 0:
        raise JckError("auroc: both classes are needed (anomalous is all True or all False)")
    # ranks from sorted positions: the number of normal scores below each anomalous one, and half of those equal to it
    neg_sorted = torch.sort(neg).values
    below = torch.searchsorted(neg_sorted, pos, right=False).to(torch.float64)
    upto = torch.searchsorted(neg_sorted, pos, right=True).to(torch.float64)
    return float((below + 0.5 * (upto - below)).sum() / (pos.numel() * neg.numel()))
