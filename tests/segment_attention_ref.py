"""Float64 restatements for the GPS tests (a helper, not a test): attention inside the segments of a row table as a plain loop over
the segments with ``torch.softmax``, ``SegmentMultiheadAttention`` around it, and ``GPSConv`` over a ``GINConv`` of
``Sequential(Linear, ReLU, Linear)`` built from a module's state dict.  Every function returns ``(out, mag)``: ``mag`` is the
magnitude sum of each output element's terms — the same chain over the absolute values of every input, weight and bias, the
softmax weights as they are; a batch norm scales it by ``|weight| / sqrt(var + eps)`` after adding the magnitude of the mean."""
import math

import torch


def _mag(t):
    return t.detach().abs()


def params_of(module):
    return {k: v.detach().double().cpu().clone() for k, v in module.state_dict().items()}


def segment_attention_ref(q, k, v, sizes, H, scale=None, vmag=None):
    n, C = q.shape
    D = C // H
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    vmag = _mag(v) if vmag is None else vmag
    out, mag, s = [q.new_zeros((0, C))], [q.new_zeros((0, C))], 0
    for m in sizes:
        qs, ks, vs, ms = (t[s:s + m].reshape(m, H, D).transpose(0, 1) for t in (q, k, v, vmag))
        p = torch.softmax(qs @ ks.transpose(1, 2) * scale, -1)
        out.append((p @ vs).transpose(0, 1).reshape(m, C))
        mag.append((p.detach() @ ms).transpose(0, 1).reshape(m, C))
        s += m
    return torch.cat(out), torch.cat(mag)


def _lin(h, s, w, b):
    return h @ w.t() + b, s @ _mag(w).t() + _mag(b)


def mha_forward(p, x, sizes, H, prefix="", xmag=None):
    """``SegmentMultiheadAttention`` (keys under ``prefix``) over rows sorted by graph."""
    C = x.shape[1]
    qkv, sqkv = _lin(x, _mag(x) if xmag is None else xmag, p[prefix + "in_proj_weight"], p[prefix + "in_proj_bias"])
    o, so = segment_attention_ref(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], sizes, H, vmag=sqkv[:, 2 * C:])
    return _lin(o, so, p[prefix + "out_proj.weight"], p[prefix + "out_proj.bias"])


def gps_forward(p, x, edge_index, sizes, H, training, taps=None):
    """``taps`` (a dict): filled with the three rows-before-a-norm tensors under the name of the bias added last to each, their
    gradients retained — a training-mode batch norm cancels that bias' gradient, the column sum of the rows' gradient."""
    def bn(h, s, name, bias=None):
        if taps is not None:
            h.retain_grad()
            taps[bias] = h
        w, b = p[name + ".module.weight"], p[name + ".module.bias"]
        mean, var = (h.mean(0), h.var(0, unbiased=False)) if training else (p[name + ".module.running_mean"],
                                                                             p[name + ".module.running_var"])
        rstd = 1.0 / torch.sqrt(var + 1e-5)
        return (h - mean) * rstd * w + b, (s + (s.mean(0) if training else _mag(mean))) * _mag(rstd * w) + _mag(b)

    src, dst = edge_index
    sx = _mag(x)
    h, s = (1 + p["conv.eps"]) * x + torch.zeros_like(x).index_add(0, dst, x[src]), \
        (1 + _mag(p["conv.eps"])) * sx + torch.zeros_like(sx).index_add(0, dst, sx[src])
    h, s = _lin(h, s, p["conv.nn.0.weight"], p["conv.nn.0.bias"])
    h, s = _lin(torch.relu(h), s, p["conv.nn.2.weight"], p["conv.nn.2.bias"])
    h1, s1 = bn(h + x, s + sx, "norm1", "conv.nn.2.bias")
    h, s = mha_forward(p, x, sizes, H, "attn.")
    h2, s2 = bn(h + x, s + sx, "norm2", "attn.out_proj.bias")
    out, so = h1 + h2, s1 + s2
    h, s = _lin(out, so, p["mlp.0.weight"], p["mlp.0.bias"])
    h, s = _lin(torch.relu(h), s, p["mlp.3.weight"], p["mlp.3.bias"])
    return bn(out + h, so + s, "norm3", "mlp.3.bias")
