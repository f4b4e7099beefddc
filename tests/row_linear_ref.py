"""float64 restatement of ``wholegraph_amd.nn.linear_rows``, its backward through torch autograd in float64, and the magnitudes the
tests' bounds are made of.

    y_pre = X[rows] @ W^T + b;   y = y_pre [y_pre > 0] if relu else y_pre
    z     = (y - mean) rstd gamma + beta   ("layer": biased variance, rstd = 1 / sqrt(var + eps))
          = y / max(||y||_2, eps)          ("l2")
          = y                              (None)
    out   = z + add

``relu_sign`` (bool, optional) replaces ``[y_pre > 0]`` where given: a test passes the kernel's own decision for the elements
whose sign float32 cannot decide (``undecided``), and leaves those elements out of the comparison of ``dy``.

Magnitudes.  ``y_terms = |X[rows]| @ |W|^T + |b|`` is the sum of the magnitudes of the terms an element of the product adds up;
a float32 product is held to ``const * y_terms``.  A gradient's ``*_terms`` are first the same plain sums for its own formula
(as tests/norm_act_ref.py returns them: ``dgamma_terms = sum_r |g| |x^|`` ...), with ``dy_terms`` in the place of ``|dy|`` where a
gradient is a product with ``dy``.  Two of the formulas have a COMPUTED factor that can be near 0 while its error is not — ``x^``
in LayerNorm's ``dgamma`` and ``dy``, ``y`` in the L2 norm's ``dy`` — so the plain sum alone would hold float32 to nothing there
(torch's own float32 backward misses the plain ``dgamma`` bound 796-fold at n = 1).  For those the first-order effect of the
product's error is ADDED, at float32 scale: the product is taken as known to ``dy_err = PRODUCT_ULPS * 2^-24 * y_terms``
(PRODUCT_ULPS: twice what torch's float32 ``F.linear`` needs on the test file's inputs, measured there on every run), and
    x^ moves by at most   xe = (2 + |x^|) max_c(dy_err) / sigma,   rstd relatively by   re = max_c(dy_err) / sigma
    dgamma:     + sum_r |g| xe
    dy (layer): + rstd (xe_c mean_c(a |x^|) + |x^_c| mean_c(a xe)) + |dy| re,     a = |g gamma|
    dy (l2):    + (e_c |g.y| + |y_c| sum_c(|g| e)) / d^3 + (|g_c| / d + 3 |y_c| |g.y| / d^3) ||e||_2 / d,     e = dy_err
all divided by ``const`` = 1e-5, so that ``const * *_terms`` is the bound.  For well-conditioned rows these additions are a few
percent of the plain sums.
"""
import torch

PRODUCT_ULPS = 11.2     # y is taken as known to PRODUCT_ULPS 2^-24 y_terms: twice the 5.6 torch's float32 F.linear needs (measured on
                        # every run by test_gpu_row_linear.py::test_gradient_bounds_are_fair_to_torch_float32)
U32 = 2.0 ** -24
CONST = 1e-5


def row_linear_ref(x, weight, bias=None, rows=None, relu=False, norm=None, gamma=None, beta=None, eps=None, add=None,
                   relu_sign=None, grad_out=None):
    """Everything in float64 on ``x``'s device; ``x`` holds the float32 rows of the input (a 16-bit table: ``table.float()``).
    Returns a dict: ``out``, ``y`` (after the ReLU, before the norm), ``y_pre``, ``y_terms``, ``xhat``, ``kappa`` [n] (the
    conditioning max(1, max_c y_terms / sqrt(var + eps)) of the row under LayerNorm), ``inv`` [n] (1 / max(||y||, eps) under
    "l2"), ``gamma`` / ``beta`` (ones / zeros where absent), ``z``, ``add``; with ``grad_out`` also ``dy``, ``dW``, ``db``,
    ``dgamma``, ``dbeta``, ``dX``, ``dadd`` and a ``*_terms`` for each."""
    dd = dict(dtype=torch.float64, device=x.device)
    if eps is None:
        eps = 1e-12 if norm == "l2" else 1e-5
    m, K = x.shape
    N = weight.shape[0]
    idx = None if rows is None else rows.long()
    xd = x.detach().double().requires_grad_(True)
    wd = weight.detach().double().requires_grad_(True)
    bd = (torch.zeros(N, **dd) if bias is None else bias.detach().double()).requires_grad_(True)
    ga = (torch.ones(N, **dd) if gamma is None or norm != "layer" else gamma.detach().double()).requires_grad_(True)
    be = (torch.zeros(N, **dd) if beta is None or norm != "layer" else beta.detach().double()).requires_grad_(True)
    ad = None if add is None else add.detach().double().requires_grad_(True)
    xr = xd if idx is None else xd[idx]
    n = xr.shape[0]
    y_pre = xr @ wd.t() + bd
    y_terms = xr.detach().abs() @ wd.detach().abs().t() + bd.detach().abs()
    sign = torch.ones(n, N, **dd)
    if relu:
        sign = ((y_pre.detach() > 0) if relu_sign is None else relu_sign).to(**dd)
    y = y_pre * sign
    yv = y.detach()
    xhat, kappa, inv = yv, torch.ones(n, **dd), torch.ones(n, **dd)
    rstd = torch.ones(n, 1, **dd)
    if norm == "layer":
        mean = y.mean(1, keepdim=True)
        var = ((y - mean) ** 2).mean(1, keepdim=True)
        rs = 1.0 / torch.sqrt(var + eps)
        xh = (y - mean) * rs
        z = xh * ga + be
        xhat, rstd = xh.detach(), rs.detach()
        kappa = torch.clamp(y_terms.amax(1, keepdim=True) * rstd, min=1.0).squeeze(1)
    elif norm == "l2":
        nrm = torch.linalg.vector_norm(y, dim=1, keepdim=True)      # (its gradient at y = 0 is 0, as F.normalize's)
        z = y / torch.clamp(nrm, min=eps)
        inv = (1.0 / torch.clamp(nrm.detach(), min=eps)).squeeze(1)
    else:
        z = y
    out = z if ad is None else z + ad
    res = dict(out=out.detach(), y=yv, y_pre=y_pre.detach(), y_terms=y_terms, xhat=xhat, kappa=kappa, inv=inv, z=z.detach(),
               gamma=ga.detach(), beta=be.detach(), add=None if ad is None else ad.detach(), norm=norm, sign=sign)
    if grad_out is None:
        return res
    g = grad_out.detach().double()
    ins = [xd, wd, bd, ga, be] + ([ad] if ad is not None else [])
    grads = torch.autograd.grad(out, ins + [y], g, allow_unused=True)
    zero = lambda gr, t: torch.zeros_like(t) if gr is None else gr      # noqa: E731
    res["dX"], res["dW"], res["db"], res["dgamma"], res["dbeta"] = (zero(gr, t) for gr, t in zip(grads[:5], ins[:5]))
    res["dadd"], res["dadd_terms"] = g, g.abs()
    res["dy"] = zero(grads[-1], yv) * sign
    ag = g.abs()
    e = PRODUCT_ULPS * U32 * y_terms
    if norm == "layer":
        a, xh = ag * ga.detach().abs(), xhat.abs()
        dy_terms = rstd * (a + a.mean(1, keepdim=True) + xh * (a * xh).mean(1, keepdim=True))
        re = e.amax(1, keepdim=True) * rstd / CONST             # (the additions of the module docstring, in units of const)
        xe = (2.0 + xh) * re
        dy_terms = dy_terms + rstd * (xe * (a * xh).mean(1, keepdim=True) + xh * (a * xe).mean(1, keepdim=True)) + res["dy"].abs() * re
        res["dgamma_terms"] = (ag * (xh + xe)).sum(0)
        res["dbeta_terms"] = ag.sum(0)
    elif norm == "l2":
        nrm = torch.sqrt((yv * yv).sum(1, keepdim=True))
        above = nrm >= eps
        safe = torch.clamp(nrm, min=1e-300)
        ya, gy = yv.abs(), (g * yv).sum(1, keepdim=True).abs()
        plain = ag / safe + ya * (ag * ya).sum(1, keepdim=True) / safe ** 3
        ec = e / CONST
        extra = (ec * gy + ya * (ag * ec).sum(1, keepdim=True)) / safe ** 3 + \
            (ag / safe + 3.0 * ya * gy / safe ** 3) * torch.sqrt((ec * ec).sum(1, keepdim=True)) / safe
        dy_terms = torch.where(above, plain + extra, ag / max(eps, 1e-300))
    else:
        dy_terms = ag
    dy_terms = dy_terms * sign
    res["dy_terms"] = dy_terms
    res["dW_terms"] = dy_terms.t() @ xr.detach().abs()
    res["db_terms"] = dy_terms.sum(0)
    gx = dy_terms @ wd.detach().abs()
    res["dX_terms"] = gx if idx is None else torch.zeros(m, K, **dd).index_add_(0, idx, gx)
    return res


def forward_bound(ref, const=1e-5):
    """The element-wise forward bound: the product's ``delta = const * y_terms`` carried through the norm.
    None:    ``delta``  (the ReLU does not enlarge it).
    "layer": ``const (|gamma_c| (2 + |x^_rc|) kappa_r + |beta_c|)`` — x^ = (y - mean) / sigma moves by at most
             (|delta_c| + mean|delta| + |x^_c| mean(|x^| |delta|)) / sigma <= (2 + |x^_c|) max_c(delta) / sigma, and
             kappa_r = max(1, max_c y_terms / sigma) also covers the float32 subtraction y - mean (|y| <= y_terms).
    "l2":    ``const ((y_terms_rc + |z_rc| ||y_terms_r||_2) / max(||y||, eps) + |z_rc|)`` — delta_c / d, the move of the norm
             (at most ||delta||_2) times |y_c| / d^2, and z's own rounding.
    ``add`` adds ``const |add_rc|``."""
    T = ref["y_terms"]
    if ref["norm"] == "layer":
        b = const * (ref["gamma"].abs() * (2.0 + ref["xhat"].abs()) * ref["kappa"].unsqueeze(1) + ref["beta"].abs())
    elif ref["norm"] == "l2":
        t2 = torch.sqrt((T * T).sum(1, keepdim=True))
        b = const * ((T + ref["z"].abs() * t2) * ref["inv"].unsqueeze(1) + ref["z"].abs())
    else:
        b = const * T
    return b if ref["add"] is None else b + const * ref["add"].abs()


def undecided(ref, const=1e-5):
    """Elements whose ReLU sign float32 does not decide: ``|y_pre| < const * y_terms``."""
    return ref["y_pre"].abs() < const * ref["y_terms"]
