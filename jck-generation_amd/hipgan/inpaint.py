"""Semantic inpainting with a trained DCGAN (Yeh et al. 2017): fit z to the KNOWN pixels of a picture through the frozen generator,
with the discriminator as a realism prior, and let G fill in the rest.  Host code - masks, the importance weighting and the final
blend are tiny; the fit itself is DcganEngine.project(weight=..., critic=...) (Sampler.inpaint).

    known = parse_mask("center:32", 64)                  # bool [64,64]: True where the picture is known
    w = importance_weights(known, window=7)              # fp32 [64,64]: known pixels weighted by the unknown share around them
    out = blend(target_u8, generated_u8, known)          # known pixels from the target, holes from G"""
import os

import torch

from ._lib import JckError

HALVES = ("left", "right", "top", "bottom")


def _check_known(known, size, what):
    k = torch.as_tensor(known)
    if k.dim() not in (2, 3) or tuple(k.shape[-2:]) != (size, size):
        raise JckError(f"{what}: a mask must be [{size},{size}] or [n,{size},{size}], got {tuple(k.shape)}")
    k = k != 0
    flat = k.reshape(-1, size * size) if k.dim() == 3 else k.reshape(1, -1)
    if not bool(flat.any(dim=1).all()):
        raise JckError(f"{what}: a mask leaves no pixel known; nothing could be fitted")
    return k


def parse_mask(spec, size):
    """The KNOWN-pixel mask, bool [S,S] (or [n,S,S] from a file), of a mask specification:
    "center:K" - a centred K x K hole, 1 <= K < S; "half:left|right|top|bottom" - that half is the hole; a path to an .npz / .npy
    file holding `mask` (non-zero = known)."""
    size = int(size)
    if size < 2:
        raise JckError(f"parse_mask: size must be >= 2, got {size}")
    if not isinstance(spec, str) or not spec:
        raise JckError(f"parse_mask: a mask specification is a non-empty string, got {spec!r}")
    if spec.startswith("center:"):
        try:
            k = int(spec[len("center:"):])
        except ValueError:
            raise JckError(f"parse_mask: {spec!r}: the hole's side must be an integer") from None
        if not 1 <= k < size:
            raise JckError(f"parse_mask: {spec!r}: the hole's side must lie in [1, {size})")
        known = torch.ones(size, size, dtype=torch.bool)
        lo = (size - k) // 2
        known[lo:lo + k, lo:lo + k] = False
        return known
    if spec.startswith("half:"):
        side = spec[len("half:"):]
        if side not in HALVES:
            raise JckError(f"parse_mask: {spec!r}: the half must be one of {', '.join(HALVES)}")
        known = torch.ones(size, size, dtype=torch.bool)
        h = size // 2
        if side == "left":
            known[:, :h] = False
        elif side == "right":
            known[:, size - h:] = False
        elif side == "top":
            known[:h, :] = False
        else:
            known[size - h:, :] = False
        return known
    if spec.endswith((".npz", ".npy")):
        import numpy as np
        if not os.path.exists(spec):
            raise JckError(f"parse_mask: {spec}: no such file")
        if spec.endswith(".npz"):
            with np.load(spec) as f:
                if "mask" not in f.files:
                    raise JckError(f"parse_mask: {spec}: no 'mask' array (found {sorted(f.files)})")
                m = f["mask"]
        else:
            m = np.load(spec)
        return _check_known(torch.from_numpy(np.ascontiguousarray(m)), size, f"parse_mask: {spec}")
    raise JckError(f"parse_mask: {spec!r} is neither 'center:K', 'half:left|right|top|bottom' nor an .npz / .npy file")


def importance_weights(known, window=7):
    """Yeh et al.'s weighting, fp32 shaped like `known`: w_p = known_p * (share of unknown pixels in the window x window neighbourhood
    of p) - an average pool with zero padding, the padding counted as known.  Known pixels close to the hole carry the fit, far ones
    nothing.  window=0: the mask itself as fp32 (every known pixel weighs 1).  window must be odd otherwise."""
    k = torch.as_tensor(known)
    if k.dim() not in (2, 3) or k.shape[-1] != k.shape[-2]:
        raise JckError(f"importance_weights: a mask must be [S,S] or [n,S,S], got {tuple(k.shape)}")
    k = (k != 0).to(torch.float32)
    window = int(window)
    if window == 0:
        return k
    if window < 1 or window % 2 == 0:
        raise JckError(f"importance_weights: window must be 0 or odd, got {window}")
    unknown = (1.0 - k).reshape(-1, 1, k.shape[-2], k.shape[-1])
    share = torch.nn.functional.avg_pool2d(unknown, window, stride=1, padding=window // 2, count_include_pad=True)
    return k * share.reshape(k.shape)


def blend(target_u8, generated_u8, known):
    """uint8 [n,S,S,3]: the target's pixels where they are known, the generator's in the holes."""
    t, g = torch.as_tensor(target_u8), torch.as_tensor(generated_u8)
    if t.dtype != torch.uint8 or g.dtype != torch.uint8 or t.dim() != 4 or t.shape != g.shape or t.shape[3] != 3:
        raise JckError(f"blend: two uint8 [n,S,S,3] batches expected, got {t.dtype} {tuple(t.shape)} and {g.dtype} {tuple(g.shape)}")
    k = _check_known(known, t.shape[1], "blend").to(t.device)
    if k.dim() == 3 and k.shape[0] != t.shape[0]:
        raise JckError(f"blend: {k.shape[0]} masks for {t.shape[0]} images")
    k = (k if k.dim() == 3 else k.unsqueeze(0)).unsqueeze(-1)
    return torch.where(k, t, g.to(t.device))
