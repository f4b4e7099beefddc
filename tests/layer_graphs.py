"""Hand-built ``LayerGraph``s shared by the GPU layer tests."""


def empty_hop_graph(n_src, seed):
    """``(lg, edge_index, destinations)``.  Hop 0: 80 destinations with 0..6 edges each; hop 1: 40 destinations and no edge.
    Destinations are distinct input rows."""
    import torch
    from wholegraph_amd import nn
    g = torch.Generator(device="cuda").manual_seed(seed)
    deg = torch.randint(0, 7, (80,), generator=g, device="cuda")
    rp0 = torch.zeros(81, dtype=torch.int32, device="cuda")
    rp0[1:] = torch.cumsum(deg, 0)
    col0 = torch.randint(0, n_src, (int(rp0[-1]),), generator=g, device="cuda", dtype=torch.int32)
    perm = torch.randperm(n_src, generator=g, device="cuda")
    h0 = nn.HopGraph(rp0, col0, perm[:80].contiguous())
    h1 = nn.HopGraph(torch.zeros(41, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"),
                     perm[80:120].contiguous())
    lg = nn.LayerGraph([h0, h1])
    ei = torch.stack([col0.long(), h0.self_rows[torch.repeat_interleave(torch.arange(80, device="cuda"), deg)]])
    return lg, ei, torch.cat([h0.self_rows, h1.self_rows])
