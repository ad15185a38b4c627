"""The reference's local gradient clipping (dgc/clip_grad.py:10-25) on a bf16 / fp16 tensor,
restated in torch CPU ops with every rounding written out: each ATen op on a 16-bit tensor
computes in fp32 and rounds to the dtype (``rdt``). test_clip16_port.py pins this to the
reference's own fixtures (tests/golden/clip16.*); the GPU tests use it as the model for
inputs the fixtures do not hold.

    x.norm(2)                 rdt(fl32(sqrt(sum x^2))), the sum in float64
    x.abs().max()             exact; NaN wins
    max_norm / (total + 1e-6) rdt(rdt(1 / rdt(total + 1e-6f)) * max_norm)  (reciprocal().mul)
    if coef < 1: x.mul_(coef) rdt(float(x) * float(coef)); a NaN coefficient leaves x alone
    x.clamp_(-v, v)           against rdt(v); a NaN element stays NaN
"""
import numpy as np
import torch

MODES = ("norm2", "norminf", "value")


def rdt(x32, dt):
    """fp32 -> dt -> fp32."""
    return x32.to(torch.float32).to(dt).to(torch.float32)


def total_norm(x, mode):
    """The 0-dim statistic as an fp32 image of the dtype's value (None for "value")."""
    if mode == "value":
        return None
    if mode == "norminf":
        a = x.float().abs()
        return torch.tensor(float("nan")) if bool(torch.isnan(a).any()) else a.max()
    d = x.double().numpy()
    with np.errstate(over="ignore", invalid="ignore"):
        root = np.float32(np.sqrt(np.sum(d * d)))
    return rdt(torch.tensor(root), x.dtype)


def coefficient(total, max_norm, dt):
    """max_norm / (total + 1e-6) on a 0-dim tensor of dtype dt (fp32 image in and out)."""
    t = rdt(total + torch.tensor(1e-6, dtype=torch.float32), dt)
    inv = rdt(torch.tensor(1.0, dtype=torch.float32) / t, dt)
    return rdt(inv * torch.tensor(max_norm, dtype=torch.float32), dt)


def clip(x, mode, param):
    """(the clipped copy of the 16-bit tensor x, total_norm, coefficient); the last two are
    fp32 images (None / the rounded bound for "value")."""
    dt = x.dtype
    if mode == "value":
        bound = rdt(torch.tensor(param, dtype=torch.float32), dt)
        return torch.clamp(x.float(), -bound, bound).to(dt), None, bound
    total = total_norm(x, mode)
    coef = coefficient(total, param, dt)
    if bool(coef < 1):   # NaN compares false
        return (x.float() * coef).to(dt), total, coef
    return x.clone(), total, coef


def f32_bits(t):
    """The fp32 bit pattern of a scalar; every NaN as the quiet NaN 0x7FC00000 (the payload
    of a NaN is not part of the reference's result: ``.item()`` gives Python's nan)."""
    x = np.float32(float(t))
    return 0x7FC00000 if np.isnan(x) else int(x.view(np.uint32))


def image(t):
    """The fp32 image of a 16-bit tensor as the fixtures store state: every NaN as 0x7FC00000."""
    a = t.detach().float().cpu().numpy().copy()
    a.view(np.uint32)[np.isnan(a)] = 0x7FC00000
    return a


def canon(b):
    """A stored fp32 bit pattern with every NaN (either sign, any payload) as 0x7FC00000."""
    return 0x7FC00000 if (b & 0x7FFFFFFF) > 0x7F800000 else b
