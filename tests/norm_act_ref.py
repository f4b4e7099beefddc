"""float64 restatement of ``wholegraph_amd.nn.norm_dropout_act`` with an explicit keep mask, its backward through torch autograd
in float64, and the magnitudes the tests' bounds are made of.

    z = x (+ residual);  y = (z - mean) rstd w + b  (biased variance, rstd = 1 / sqrt(var + eps));  out = y * gate
    gate = keep / (1 - p) * [y > 0]      (a constant of the backward)

``relu_sign`` (bool, optional) replaces ``[y > 0]`` where given: a test passes the kernel's own decision for the elements whose
sign float32 cannot decide (``undecided``), and leaves those elements out of the comparison.
"""
import torch


def norm_act_ref(x, residual=None, weight=None, bias=None, keep=None, p=0.0, norm=True, relu=True, eps=1e-5, relu_sign=None,
                 grad_out=None):
    """Everything in float64 on ``x``'s device.  Returns a dict: ``out``, ``y`` (before the gate), ``xhat``, ``kappa`` [n] (the
    conditioning max(1, max_c |z| / sqrt(var + eps)) of z - mean in float32), ``w`` / ``b`` (ones / zeros where absent); with
    ``grad_out`` also ``dz``, ``dw``, ``db`` (autograd) and ``dz_terms``, ``dw_terms``, ``db_terms`` (the sums of the
    magnitudes of the terms each gradient element adds up)."""
    dd = dict(dtype=torch.float64, device=x.device)
    n, C = x.shape
    xd = x.detach().double().requires_grad_(True)
    rd = None if residual is None else residual.detach().double().requires_grad_(True)
    w = torch.ones(C, **dd) if weight is None or not norm else weight.detach().double()
    b = torch.zeros(C, **dd) if bias is None or not norm else bias.detach().double()
    w.requires_grad_(True), b.requires_grad_(True)
    z = xd if rd is None else xd + rd
    if norm:
        mean = z.mean(1, keepdim=True)
        var = ((z - mean) ** 2).mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(var + eps)
        xhat = (z - mean) * rstd
        y = xhat * w + b
        kappa = torch.clamp(z.detach().abs().amax(1, keepdim=True) * rstd.detach(), min=1.0).squeeze(1) if C else torch.ones(n, **dd)
    else:
        rstd, xhat, y, kappa = torch.ones(n, 1, **dd), z, z, torch.ones(n, **dd)
    gate = torch.ones(n, C, **dd)
    if p > 0:
        gate = keep.to(**dd) / (1.0 - p) if p < 1 else torch.zeros(n, C, **dd)
    if relu:
        sign = y.detach() > 0
        if relu_sign is not None:
            sign = relu_sign
        gate = gate * sign.to(**dd)
    out = y * gate
    res = dict(out=out.detach(), y=y.detach(), xhat=xhat.detach(), kappa=kappa, w=w.detach(), b=b.detach(), gate=gate)
    if grad_out is not None:
        g = grad_out.detach().double()
        ins = [xd, w, b] + ([rd] if rd is not None else [])
        grads = torch.autograd.grad(out, ins, g, allow_unused=True)
        zero = lambda t, like: torch.zeros_like(like) if t is None else t      # noqa: E731
        res["dz"], res["dw"], res["db"] = zero(grads[0], xd), zero(grads[1], w), zero(grads[2], b)
        if rd is not None:
            res["dres"] = zero(grads[3], rd)
        gy = (g * gate).abs()
        if norm:
            a, xh = gy * w.detach().abs(), xhat.detach().abs()
            res["dz_terms"] = rstd.detach() * (a + a.mean(1, keepdim=True) + xh * (a * xh).mean(1, keepdim=True))
            res["dw_terms"], res["db_terms"] = (gy * xh).sum(0), gy.sum(0)
        else:
            res["dz_terms"] = gy
    return res


def forward_bound(ref, p=0.0, const=1e-5):
    """The element-wise forward bound: ``const (|w_c| (1 + |x^_rc|) kappa_r + |b_c|) / (1 - p)``."""
    scale = 1.0 / (1.0 - p) if p < 1 else 1.0
    return const * (ref["w"].abs() * (1.0 + ref["xhat"].abs()) * ref["kappa"].unsqueeze(1) + ref["b"].abs()) * scale


def undecided(ref, const=1e-5):
    """Elements whose ReLU sign float32 does not decide: ``|y| < const (|w_c| + |b_c|)``."""
    return ref["y"].abs() < const * (ref["w"].abs() + ref["b"].abs())
