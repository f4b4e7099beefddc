"""A plain float64 restatement of one segment of the grouped Linear (``wholegraph_amd.nn.grouped_linear``, ``HeteroLinear``,
``HeteroDictLinear``):  out = act(x[rows] @ W + b + add), with every gradient against ``grad_out`` and, beside each value, the sum
of the magnitudes of the terms it is a sum of — what the project's bound ``|got - ref| <= 1e-5 x sum|terms|`` is taken of."""
import torch


def grouped_linear_ref(x, w, b, add, grad_out, layout="nk", rows=None, mask=None):
    """``x`` [m, K], ``w`` [N, K] ("nk") or [K, N] ("kn"), ``b`` [N] or None, ``add`` [n, N] or None, ``grad_out`` [n, N],
    ``rows`` (ids into x, repeats allowed) or None, ``mask`` (bool [n, N]: where the ReLU lets a value through) or None = no
    ReLU.  Returns a dict of float64 tensors: ``out``, ``dx`` (of the whole ``x``), ``dw`` (in ``w``'s layout), ``db``, ``dadd``
    and ``<name>_terms`` for each."""
    d = lambda t: None if t is None else t.detach().double().cpu()      # noqa: E731
    x, w, b, add, go = d(x), d(w), d(b), d(add), d(grad_out)
    wm = w.t() if layout == "nk" else w                                # [K, N]
    xr = x if rows is None else x[rows.cpu().long()]
    y, terms = xr @ wm, xr.abs() @ wm.abs()
    if b is not None:
        y, terms = y + b, terms + b.abs()
    if add is not None:
        y, terms = y + add, terms + add.abs()
    keep = torch.ones_like(y) if mask is None else mask.cpu().double()
    dy = go * keep
    dxr, dxr_terms = dy @ wm.t(), dy.abs() @ wm.abs().t()
    if rows is not None:
        idx = rows.cpu().long()
        dxr, dxr_terms = torch.zeros_like(x).index_add_(0, idx, dxr), torch.zeros_like(x).index_add_(0, idx, dxr_terms)
    dw, dw_terms = xr.t() @ dy, xr.abs().t() @ dy.abs()
    if layout == "nk":
        dw, dw_terms = dw.t(), dw_terms.t()
    return dict(out=y * keep, out_terms=terms, dx=dxr, dx_terms=dxr_terms, dw=dw, dw_terms=dw_terms, db=dy.sum(0),
                db_terms=dy.abs().sum(0), dadd=dy, dadd_terms=dy.abs())
