"""The MLP edge decoder of ``wholegraph_amd.nn.pair_mlp`` restated in float64, with the magnitude sums its tests' bars are
built from (shared by tests/test_link_mlp_host.py and tests/test_gpu_link_mlp_head.py; no test in here)."""


def reference(x_src, x_dst, index, w1, b1, w2, b2):
    """``(s, z, m, M)`` in float64 for the pairs ``index`` [2, P] (all in range):
    ``a_p = [x_src[i_p] | x_dst[j_p]]``, ``z_p = a_p W1^T + b1``, ``s_p = relu(z_p) . w2 + b2``,
    ``m_pn = sum_k |a_pk W1_nk| + |b1_n|``, ``M_p = sum_n |w2_n| m_pn + |b2|``.  ``b1`` / ``b2`` may be None."""
    import torch
    a = torch.cat([x_src.detach().double()[index[0]], x_dst.detach().double()[index[1]]], dim=1)
    w1, w2 = w1.detach().double(), w2.detach().double().reshape(-1)
    z = a @ w1.t()
    m = a.abs() @ w1.abs().t()
    if b1 is not None:
        z = z + b1.detach().double()
        m = m + b1.detach().double().abs()
    s = z.clamp(min=0) @ w2
    M = m @ w2.abs()
    if b2 is not None:
        s = s + b2.detach().double().reshape(())
        M = M + b2.detach().double().abs().reshape(())
    return s, z, m, M
